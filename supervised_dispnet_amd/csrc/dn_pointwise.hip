// HBM-bound NHWC kernels around the convolutions that are neither BatchNorm (dn_bn.hip) nor an optimizer (dn_optim.hip): activation
// backward with bias-gradient column sums and their finalize, the plain max-pools (2x2 backward, 3x3 / stride 2), nearest / bilinear
// upsamples, the reflection-pad fold, the spatial mean, (x - sub) / div, reciprocal, fill, copy.  gfx950 only.
// The column reductions are the two-stage ones of dn_colreduce.h.
#include "dn_colreduce.h"

namespace dn {

// gradient of the plain 2x2 max-pool: every input pixel of a window gets the window's gradient if it was the arg-max, else 0
__global__ void __launch_bounds__(kThreads) maxpool2_bwd_kernel(const float* __restrict__ dpooled, const uint8_t* __restrict__ idx, int N, int H,
                                                                int W, int C, float* __restrict__ dx, int accumulate) {
  const int PH = H / 2, PW = W / 2, G = C / 4;
  const long long total = (long long)N * PH * PW * G;
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int g = (int)(i % G);
    long long pix = i / G;
    const int px = (int)(pix % PW);
    pix /= PW;
    const int py = (int)(pix % PH), n = (int)(pix / PH);
    const uchar4 code = *reinterpret_cast<const uchar4*>(idx + i * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(dpooled + i * 4);
    float* base = dx + (((long long)n * H + 2 * py) * W + 2 * px) * C + g * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float* dst = base + ((long long)(q >> 1) * W + (q & 1)) * C;
      f32x4 o = accumulate ? *reinterpret_cast<const f32x4*>(dst) : f32x4{0.f, 0.f, 0.f, 0.f};
      if ((code.x & 3) == q) o[0] += gv[0];
      if ((code.y & 3) == q) o[1] += gv[1];
      if ((code.z & 3) == q) o[2] += gv[2];
      if ((code.w & 3) == q) o[3] += gv[3];
      *reinterpret_cast<f32x4*>(dst) = o;
    }
  }
}

struct ActBwdOp {
  static constexpr int NACC = 1;
  const float* src;      // == g: in place
  float* g;
  const float* y_post;
  int act;
  float p0, p1;
  int C;
  template <int V>
  __device__ __forceinline__ void apply(long long row, int c0, float (&acc)[V][1]) const {
    const long long o = row * C + c0;
    Vec<V> gv = ldv<V>(src + o);
    if (act == DN_ACT_NONE) {
      if (src != g) stv<V>(g + o, gv);
    } else {
      const Vec<V> yv = ldv<V>(y_post + o);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float yp = yv.v[e];
        float d = 1.f;
        if (act == DN_ACT_RELU) d = yp > 0.f ? 1.f : 0.f;
        else if (act == DN_ACT_LEAKY) d = yp > 0.f ? 1.f : p0;
        else if (act == DN_ACT_ELU) d = yp > 0.f ? 1.f : (yp + 1.f);
        else if (act == DN_ACT_SIGMOID_AFFINE) {
          const float sg = (yp - p1) / p0;
          d = p0 * sg * (1.f - sg);
        }
        gv.v[e] *= d;
      }
      stv<V>(g + o, gv);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e][0] += gv.v[e];
  }
};

// out[c] = sum_rows partial[(row*C + c)*stride + offset].  One 64-lane wave per channel: lanes stride over the rows
// (fp64 accumulation), wave-shuffle reduction -- the row count is up to 1024, so a serial per-thread loop is latency-bound.
__global__ void __launch_bounds__(256) colsum_finalize_kernel(const float* __restrict__ partial, int rows, int C, int stride, int offset,
                                                              float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  double s = 0.0;
  for (int r = lane; r < rows; r += 64) s += (double)partial[((long long)r * C + c) * stride + offset];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) out[c] = (float)s;
}

// ----------------------------------------------------------------------------------------- MaxPool 3x3 / stride 2 / pad 1
__global__ void __launch_bounds__(kThreads) maxpool3s2_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C, int OH, int OW,
                                                                  float* __restrict__ out, uint8_t* __restrict__ idx) {
  const int G = C / 4;
  const long long total = (long long)N * OH * OW * G;
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int g = (int)(i % G);
    long long pix = i / G;
    const int ox = (int)(pix % OW);
    pix /= OW;
    const int oy = (int)(pix % OH), n = (int)(pix / OH);
    f32x4 best = f32x4{-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    int bi[4] = {0, 0, 0, 0};
    bool any = false;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const int iy = 2 * oy - 1 + q / 3, ix = 2 * ox - 1 + q % 3;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((long long)n * H + iy) * W + ix) * C + g * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (!any || v[e] > best[e]) {
          best[e] = v[e];
          bi[e] = q;
        }
      any = true;
    }
    *reinterpret_cast<f32x4*>(out + i * 4) = best;
    uchar4 code;
    code.x = (uint8_t)bi[0]; code.y = (uint8_t)bi[1]; code.z = (uint8_t)bi[2]; code.w = (uint8_t)bi[3];
    *reinterpret_cast<uchar4*>(idx + i * 4) = code;
  }
}

__global__ void __launch_bounds__(kThreads) maxpool3s2_bwd_kernel(const float* __restrict__ dout, const uint8_t* __restrict__ idx, int N, int H,
                                                                  int W, int C, int OH, int OW, float* __restrict__ dx, int accumulate) {
  const int G = C / 4;
  const long long total = (long long)N * H * W * G;
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int g = (int)(i % G);
    long long pix = i / G;
    const int ix = (int)(pix % W);
    pix /= W;
    const int iy = (int)(pix % H), n = (int)(pix / H);
    f32x4 s = accumulate ? *reinterpret_cast<const f32x4*>(dx + i * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    // windows (oy, ox) with 2*oy - 1 <= iy <= 2*oy + 1
    for (int oy = (iy) / 2; oy <= (iy + 1) / 2; ++oy) {
      if (oy < 0 || oy >= OH) continue;
      const int qy = iy - (2 * oy - 1);
      for (int ox = (ix) / 2; ox <= (ix + 1) / 2; ++ox) {
        if (ox < 0 || ox >= OW) continue;
        const int q = qy * 3 + (ix - (2 * ox - 1));
        const long long o = ((((long long)n * OH + oy) * OW + ox) * G + g) * 4;
        const uchar4 code = *reinterpret_cast<const uchar4*>(idx + o);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(dout + o);
        if (code.x == q) s[0] += gv[0];
        if (code.y == q) s[1] += gv[1];
        if (code.z == q) s[2] += gv[2];
        if (code.w == q) s[3] += gv[3];
      }
    }
    *reinterpret_cast<f32x4*>(dx + i * 4) = s;
  }
}

// backward of nearest x2 upsample for NHWC with C channels
__global__ void upsample2x_nearest_bwd_nhwc_kernel(const float* __restrict__ dfull, int N, int h, int w, int C, float* __restrict__ dlow,
                                                   int accumulate) {
  const long long total = (long long)N * h * w * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    long long t = i / C;
    const int x = (int)(t % w);
    t /= w;
    const int yy = (int)(t % h), n = (int)(t / h);
    const float* b = dfull + ((((long long)n * 2 * h + 2 * yy) * 2 * w + 2 * x) * C + c);
    const long long rs = (long long)2 * w * C;
    float s = (b[0] + b[C]) + (b[rs] + b[rs + C]);
    if (accumulate) s += dlow[i];
    dlow[i] = s;
  }
}

// dx[n][y][x][c] (+)= sum over padded (py, px) in [-pad, H+pad) x [-pad, W+pad) with reflect(py) == y, reflect(px) == x
__global__ void reflect_fold_kernel(const float* __restrict__ dxp, int N, int H, int W, int C, int pad, float* __restrict__ dx, int accumulate) {
  const long long total = (long long)N * H * W * C;
  const int PH = H + 2 * pad, PW = W + 2 * pad;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    long long t = i / C;
    const int x = (int)(t % W);
    t /= W;
    const int y = (int)(t % H), n = (int)(t / H);
    int ys[3], xs[3], ny = 0, nx = 0;
    ys[ny++] = y;
    if (y >= 1 && y <= pad) ys[ny++] = -y;
    if (y <= H - 2 && y >= H - 1 - pad) ys[ny++] = 2 * (H - 1) - y;
    xs[nx++] = x;
    if (x >= 1 && x <= pad) xs[nx++] = -x;
    if (x <= W - 2 && x >= W - 1 - pad) xs[nx++] = 2 * (W - 1) - x;
    float s = accumulate ? dx[i] : 0.f;
    for (int a = 0; a < ny; ++a)
      for (int b = 0; b < nx; ++b) s += dxp[(((long long)n * PH + ys[a] + pad) * PW + xs[b] + pad) * C + c];
    dx[i] = s;
  }
}

// out[n][c] = scale * mean over the HW pixels of x[n][p][c]   (pose = 0.01 * pose_pred.mean(3).mean(2), models/PoseExpNet.py:73-75)
// one block per sample; threads stride over (pixel, channel) so consecutive lanes read consecutive addresses
__global__ void __launch_bounds__(kThreads) spatial_mean_fwd_kernel(const float* __restrict__ x, long long HW, int C, float scale,
                                                                    float* __restrict__ out) {
  const int n = blockIdx.x;
  const float* X = x + (long long)n * HW * C;
  __shared__ float red[kThreads];
  for (int c0 = 0; c0 < C; c0 += kThreads) {
    // thread t handles channel c0 + (t % cw) for pixels t / cw, t / cw + stride, ...
    const int cw = (C - c0) < kThreads ? (C - c0) : kThreads;
    const int lanes_per_c = kThreads / cw;
    const int c = threadIdx.x % cw, pl = threadIdx.x / cw;
    float s = 0.f;
    if (pl < lanes_per_c)
      for (long long p = pl; p < HW; p += lanes_per_c) s += X[p * C + c0 + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < cw) {
      float t = 0.f;
      for (int q = 0; q < lanes_per_c; ++q) t += red[q * cw + threadIdx.x];
      out[(long long)n * C + c0 + threadIdx.x] = scale * (t / (float)HW);
    }
    __syncthreads();
  }
}

__global__ void spatial_mean_bwd_kernel(const float* __restrict__ dout, int N, long long HW, int C, float scale, float* __restrict__ dx) {
  const long long total = (long long)N * HW * C;
  const float k = scale / (float)HW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long long n = i / (HW * C);
    dx[i] = dout[n * C + c] * k;
  }
}

__global__ void sub_div_kernel(const float* __restrict__ x, long long n, float sub, float div, float* __restrict__ out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = (x[i] - sub) / div;
}

// ----------------------------------------------------------------------------------------------- 1-channel helpers
__global__ void upsample2x_nearest_bwd_kernel(const float* __restrict__ dfull, int N, int h, int w, float* __restrict__ dlow, int accumulate) {
  const long long total = (long long)N * h * w;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % w);
    const long long t = i / w;
    const int yy = (int)(t % h), n = (int)(t / h);
    const float* b = dfull + (((long long)n * 2 * h + 2 * yy) * 2 * w + 2 * x);
    float s = (b[0] + b[1]) + (b[2 * w] + b[2 * w + 1]);
    if (accumulate) s += dlow[i];
    dlow[i] = s;
  }
}

__device__ __forceinline__ void bilin_src(int o, int in_size, int* i0, int* i1, float* l1) {
  float src = 0.5f * ((float)o + 0.5f) - 0.5f;   // scale 1/2, align_corners = False
  if (src < 0.f) src = 0.f;
  int a = (int)src;
  if (a > in_size - 1) a = in_size - 1;
  *i0 = a;
  *i1 = a + (a < in_size - 1 ? 1 : 0);
  *l1 = src - (float)a;
}

__global__ void upsample2x_bilinear_fwd_kernel(const float* __restrict__ low, int N, int h, int w, int OH, int OW, float* __restrict__ out) {
  const long long total = (long long)N * OH * OW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % OW);
    const long long t = i / OW;
    const int oy = (int)(t % OH), n = (int)(t / OH);
    int y0, y1, x0, x1;
    float ly, lx;
    bilin_src(oy, h, &y0, &y1, &ly);
    bilin_src(ox, w, &x0, &x1, &lx);
    const float* b = low + (long long)n * h * w;
    const float hy = 1.f - ly, hx = 1.f - lx;
    out[i] = hy * (hx * b[y0 * w + x0] + lx * b[y0 * w + x1]) + ly * (hx * b[y1 * w + x0] + lx * b[y1 * w + x1]);
  }
}

__global__ void upsample2x_bilinear_bwd_kernel(const float* __restrict__ dout, int N, int h, int w, int OH, int OW, float* __restrict__ dlow,
                                               int accumulate) {
  const long long total = (long long)N * h * w;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % w);
    const long long t = i / w;
    const int yy = (int)(t % h), n = (int)(t / h);
    const float* g = dout + (long long)n * OH * OW;
    float s = 0.f;
    for (int oy = 2 * yy - 2; oy <= 2 * yy + 2; ++oy) {
      if (oy < 0 || oy >= OH) continue;
      int y0, y1;
      float ly;
      bilin_src(oy, h, &y0, &y1, &ly);
      float wy = 0.f;
      if (y0 == yy) wy += 1.f - ly;
      if (y1 == yy) wy += ly;
      if (wy == 0.f) continue;
      for (int ox = 2 * x - 2; ox <= 2 * x + 2; ++ox) {
        if (ox < 0 || ox >= OW) continue;
        int x0, x1;
        float lx;
        bilin_src(ox, w, &x0, &x1, &lx);
        float wx = 0.f;
        if (x0 == x) wx += 1.f - lx;
        if (x1 == x) wx += lx;
        if (wx != 0.f) s += wy * wx * g[(long long)oy * OW + ox];
      }
    }
    if (accumulate) s += dlow[i];
    dlow[i] = s;
  }
}

__global__ void reciprocal_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) y[i] = 1.f / x[i];
}
__global__ void reciprocal_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float v = y[i];
    dx[i] = -dy[i] * v * v;
  }
}

__global__ void fill_kernel(float* __restrict__ p, float v, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}

}  // namespace dn

using namespace dn;

extern "C" {

int32_t dn_reduce_blocks(int64_t rows, int32_t C) { return reduce_blocks(rows, C); }

int dn_maxpool2_bwd(const float* dpooled, const uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, float* dx, int32_t accumulate,
                    dn_stream_t stream) {
  DN_REQUIRE(dpooled && idx && dx && N > 0, DN_ERR_BAD_ARG, "dn_maxpool2_bwd: bad argument");
  DN_REQUIRE(C % 4 == 0 && H % 2 == 0 && W % 2 == 0, DN_ERR_UNSUPPORTED, "dn_maxpool2_bwd: need C%%4==0 and even H,W");
  const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
  DN_LAUNCH(maxpool2_bwd_kernel, dim3(ew_blocks(total)), dim3(kThreads), 0, as_stream(stream), dpooled, idx, N, H, W, C, dx, accumulate);
  return check_launch("maxpool2_bwd_kernel");
}

int dn_act_bwd_reduce(float* g, const float* y_post, int32_t act, float p0, float p1, int64_t rows, int32_t C, float* partial,
                      dn_stream_t stream) {
  DN_REQUIRE(g && partial && rows > 0 && C > 0 && (act == DN_ACT_NONE || y_post), DN_ERR_BAD_ARG, "dn_act_bwd_reduce: bad argument");
  ActBwdOp op{g, g, y_post, act, p0, p1, C};
  return launch_colreduce(op, rows, C, partial, as_stream(stream), "act_bwd_reduce");
}

// out of place: g_out = g_in * act'(.) -- the incoming gradient is the framework's tensor and must not be written (engine.seed_grad used to
// copy it first: one more launch on the critical stream)
int dn_act_bwd_reduce_from(const float* g_in, float* g_out, const float* y_post, int32_t act, float p0, float p1, int64_t rows, int32_t C,
                           float* partial, dn_stream_t stream) {
  DN_REQUIRE(g_in && g_out && partial && rows > 0 && C > 0 && (act == DN_ACT_NONE || y_post), DN_ERR_BAD_ARG, "dn_act_bwd_reduce_from: bad argument");
  ActBwdOp op{g_in, g_out, y_post, act, p0, p1, C};
  return launch_colreduce(op, rows, C, partial, as_stream(stream), "act_bwd_reduce_from");
}

int dn_colsum_finalize(const float* partial, int32_t rows, int32_t C, int32_t stride, int32_t offset, float* out, dn_stream_t stream) {
  DN_REQUIRE(partial && out && rows > 0 && C > 0 && stride > 0 && offset >= 0 && offset < stride, DN_ERR_BAD_ARG, "dn_colsum_finalize: bad argument");
  DN_LAUNCH(colsum_finalize_kernel, dim3((C + 3) / 4), dim3(256), 0, as_stream(stream), partial, rows, C, stride, offset, out);
  return check_launch("colsum_finalize_kernel");
}

int dn_upsample2x_nearest_bwd(const float* dfull, int32_t N, int32_t h, int32_t w, float* dlow, int32_t accumulate, dn_stream_t stream) {
  DN_REQUIRE(dfull && dlow && N > 0 && h > 0 && w > 0, DN_ERR_BAD_ARG, "dn_upsample2x_nearest_bwd: bad argument");
  DN_LAUNCH(upsample2x_nearest_bwd_kernel, dim3(ew_blocks((long long)N * h * w)), dim3(256), 0, as_stream(stream), dfull, N, h, w,
                     dlow, accumulate);
  return check_launch("upsample2x_nearest_bwd_kernel");
}

int dn_upsample2x_bilinear_fwd(const float* low, int32_t N, int32_t h, int32_t w, int32_t OH, int32_t OW, float* out, dn_stream_t stream) {
  DN_REQUIRE(low && out && N > 0 && OH <= 2 * h && OW <= 2 * w && OH > 0 && OW > 0, DN_ERR_BAD_ARG, "dn_upsample2x_bilinear_fwd: bad argument");
  DN_LAUNCH(upsample2x_bilinear_fwd_kernel, dim3(ew_blocks((long long)N * OH * OW)), dim3(256), 0, as_stream(stream), low, N, h, w,
                     OH, OW, out);
  return check_launch("upsample2x_bilinear_fwd_kernel");
}

int dn_upsample2x_bilinear_bwd(const float* dout, int32_t N, int32_t h, int32_t w, int32_t OH, int32_t OW, float* dlow, int32_t accumulate,
                               dn_stream_t stream) {
  DN_REQUIRE(dout && dlow && N > 0 && OH <= 2 * h && OW <= 2 * w && OH > 0 && OW > 0, DN_ERR_BAD_ARG, "dn_upsample2x_bilinear_bwd: bad argument");
  DN_LAUNCH(upsample2x_bilinear_bwd_kernel, dim3(ew_blocks((long long)N * h * w)), dim3(256), 0, as_stream(stream), dout, N, h, w,
                     OH, OW, dlow, accumulate);
  return check_launch("upsample2x_bilinear_bwd_kernel");
}

int32_t dn_maxpool3s2_out(int32_t H, int32_t ceil_mode) {
  if (!ceil_mode) return (H - 1) / 2 + 1;                  // floor((H + 2 - 3) / 2) + 1
  int o = H / 2 + 1;                                        // ceil((H - 1) / 2) + 1
  if ((o - 1) * 2 >= H + 1) --o;                            // (ATen: the last window must start inside the input or its left padding)
  return o;
}

int dn_maxpool3s2_fwd(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ceil_mode, float* out, uint8_t* idx, dn_stream_t stream) {
  DN_REQUIRE(x && out && idx && N > 0 && H > 0 && W > 0, DN_ERR_BAD_ARG, "dn_maxpool3s2_fwd: bad argument");
  DN_REQUIRE(C % 4 == 0, DN_ERR_UNSUPPORTED, "dn_maxpool3s2_fwd: need C%%4==0");
  const int OH = dn_maxpool3s2_out(H, ceil_mode), OW = dn_maxpool3s2_out(W, ceil_mode);
  DN_LAUNCH(maxpool3s2_fwd_kernel, dim3(ew_blocks((long long)N * OH * OW * (C / 4))), dim3(kThreads), 0, as_stream(stream), x, N, H, W,
                     C, OH, OW, out, idx);
  return check_launch("maxpool3s2_fwd_kernel");
}

int dn_maxpool3s2_bwd(const float* dout, const uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ceil_mode, float* dx,
                      int32_t accumulate, dn_stream_t stream) {
  DN_REQUIRE(dout && idx && dx && N > 0 && H > 0 && W > 0, DN_ERR_BAD_ARG, "dn_maxpool3s2_bwd: bad argument");
  DN_REQUIRE(C % 4 == 0, DN_ERR_UNSUPPORTED, "dn_maxpool3s2_bwd: need C%%4==0");
  const int OH = dn_maxpool3s2_out(H, ceil_mode), OW = dn_maxpool3s2_out(W, ceil_mode);
  DN_LAUNCH(maxpool3s2_bwd_kernel, dim3(ew_blocks((long long)N * H * W * (C / 4))), dim3(kThreads), 0, as_stream(stream), dout, idx, N, H,
                     W, C, OH, OW, dx, accumulate);
  return check_launch("maxpool3s2_bwd_kernel");
}

int dn_upsample2x_nearest_bwd_nhwc(const float* dfull, int32_t N, int32_t h, int32_t w, int32_t C, float* dlow, int32_t accumulate,
                                   dn_stream_t stream) {
  DN_REQUIRE(dfull && dlow && N > 0 && h > 0 && w > 0 && C > 0, DN_ERR_BAD_ARG, "dn_upsample2x_nearest_bwd_nhwc: bad argument");
  DN_LAUNCH(upsample2x_nearest_bwd_nhwc_kernel, dim3(ew_blocks((long long)N * h * w * C)), dim3(256), 0, as_stream(stream), dfull, N, h,
                     w, C, dlow, accumulate);
  return check_launch("upsample2x_nearest_bwd_nhwc_kernel");
}

int dn_reflect_fold(const float* dxp, int32_t N, int32_t H, int32_t W, int32_t C, int32_t pad, float* dx, int32_t accumulate, dn_stream_t stream) {
  DN_REQUIRE(dxp && dx && N > 0 && C > 0 && pad >= 1 && H > pad && W > pad, DN_ERR_BAD_ARG, "dn_reflect_fold: bad argument (needs H, W > pad)");
  DN_LAUNCH(reflect_fold_kernel, dim3(ew_blocks((long long)N * H * W * C)), dim3(256), 0, as_stream(stream), dxp, N, H, W, C, pad, dx,
                     accumulate);
  return check_launch("reflect_fold_kernel");
}

int dn_sub_div(const float* x, int64_t n, float sub, float div, float* out, dn_stream_t stream) {
  DN_REQUIRE(x && out && n > 0 && div != 0.f, DN_ERR_BAD_ARG, "dn_sub_div: bad argument");
  DN_LAUNCH(sub_div_kernel, dim3(ew_blocks(n)), dim3(256), 0, as_stream(stream), x, (long long)n, sub, div, out);
  return check_launch("sub_div_kernel");
}

int dn_spatial_mean_fwd(const float* x, int32_t N, int64_t HW, int32_t C, float scale, float* out, dn_stream_t stream) {
  DN_REQUIRE(x && out && N > 0 && HW > 0 && C > 0, DN_ERR_BAD_ARG, "dn_spatial_mean_fwd: bad argument");
  DN_LAUNCH(spatial_mean_fwd_kernel, dim3(N), dim3(kThreads), 0, as_stream(stream), x, (long long)HW, C, scale, out);
  return check_launch("spatial_mean_fwd_kernel");
}

int dn_spatial_mean_bwd(const float* dout, int32_t N, int64_t HW, int32_t C, float scale, float* dx, dn_stream_t stream) {
  DN_REQUIRE(dout && dx && N > 0 && HW > 0 && C > 0, DN_ERR_BAD_ARG, "dn_spatial_mean_bwd: bad argument");
  DN_LAUNCH(spatial_mean_bwd_kernel, dim3(ew_blocks((long long)N * HW * C)), dim3(256), 0, as_stream(stream), dout, N, (long long)HW, C,
                     scale, dx);
  return check_launch("spatial_mean_bwd_kernel");
}

int dn_reciprocal_fwd(const float* x, float* y, int64_t n, dn_stream_t stream) {
  DN_REQUIRE(x && y && n > 0, DN_ERR_BAD_ARG, "dn_reciprocal_fwd: bad argument");
  DN_LAUNCH(reciprocal_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, as_stream(stream), x, y, (long long)n);
  return check_launch("reciprocal_fwd_kernel");
}

int dn_reciprocal_bwd(const float* dy, const float* y, float* dx, int64_t n, dn_stream_t stream) {
  DN_REQUIRE(dy && y && dx && n > 0, DN_ERR_BAD_ARG, "dn_reciprocal_bwd: bad argument");
  DN_LAUNCH(reciprocal_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, as_stream(stream), dy, y, dx, (long long)n);
  return check_launch("reciprocal_bwd_kernel");
}

int dn_fill(float* p, float value, int64_t n, dn_stream_t stream) {
  DN_REQUIRE(p && n >= 0, DN_ERR_BAD_ARG, "dn_fill: bad argument");
  if (n == 0) return DN_OK;
  DN_LAUNCH(fill_kernel, dim3(ew_blocks(n)), dim3(256), 0, as_stream(stream), p, value, (long long)n);
  return check_launch("fill_kernel");
}

__global__ void __launch_bounds__(256) copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = src[i];
}

int dn_copy(const float* src, float* dst, int64_t n, dn_stream_t stream) {
  DN_REQUIRE(src && dst && n >= 0, DN_ERR_BAD_ARG, "dn_copy: bad argument");
  if (n == 0) return DN_OK;
  DN_LAUNCH(copy_kernel, dim3(ew_blocks(n)), dim3(256), 0, as_stream(stream), src, dst, (long long)n);
  return check_launch("copy_kernel");
}

}  // extern "C"
