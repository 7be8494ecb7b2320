// monodepth2's depth evaluation (evaluate_depth.py) on the device, between the network's disparity and the seven error numbers of an
// image (the contracts are written out in include/dispnet_hip.h):
//   dn_mono2_post_process     batch_post_process_disparity: the prediction blended with that of the mirrored frame, which is read
//                             mirrored (no un-flip pass), by the two 5 %-wide border ramps; fp64 from the fp32 inputs, one rounding;
//   dn_bilinear_recip_ragged  cv2.resize(disp, (W_b, H_b)) (INTER_LINEAR: half-pixel centres, replicated edges, no antialiasing) to a
//                             per-image ground-truth size in fp64, then depth = 1 / disp, one rounding to fp32, written into the ragged
//                             layout of dn_zoom3_clip;
//   dn_eval_errors_clamp      dn_eval_errors with the order of monodepth2: median ratio of the unclamped depth, scale, clamp to [lo, hi],
//                             metrics.  Selection and sums are dn_eval_errors.h's.
// All three are one pass over their map: a thread makes four consecutive outputs and stores them as 16 bytes where the addresses allow.
#include "dn_internal.h"
#include "dn_eval_errors.h"

#pragma clang fp contract(off)

namespace dn {

constexpr int kM2Threads = 256;
constexpr int kM2MaxBlocks = 2048;       // grid-stride beyond this

static __device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the left ramp lm at column x of w >= 2 columns: 1 - clip(20 * (x / (w - 1) - 0.05), 0, 1)
static __device__ __forceinline__ double left_ramp(int x, int w) {
  const double l = (double)x / (double)(w - 1);
  return 1.0 - fmin(fmax(20.0 * (l - 0.05), 0.0), 1.0);
}

static __device__ __forceinline__ float post_process_pixel(float Lf, float Rf, int x, int w) {
  const double lm = left_ramp(x, w), rm = left_ramp(w - 1 - x, w);
  const double L = (double)Lf, R = (double)Rf;
  return (float)(rm * L + lm * R + (1.0 - lm - rm) * (0.5 * (L + R)));
}

// disp [2B][h][w]: plane b and the mirrored read of plane B + b -> out [B][h][w].  kVec: w % 4 == 0 and both bases 16-byte aligned; a
// thread takes columns x .. x + 3 of one row, whose mirrored partners w - 4 - x .. w - 1 - x are one aligned float4 too.
template <bool kVec>
__global__ void __launch_bounds__(kM2Threads) mono2_post_process_kernel(const float* __restrict__ disp, int B, int h, int w,
                                                                        float* __restrict__ out) {
  const long long plane = (long long)h * w, half = (long long)B * plane;
  if (kVec) {
    const int wq = w >> 2;
    const long long total = (long long)B * h * wq;
    for (long long t = blockIdx.x * (long long)kM2Threads + threadIdx.x; t < total; t += (long long)gridDim.x * kM2Threads) {
      const int x = (int)(t % wq) * 4;
      const long long row = (t / wq) * w;                // element offset of the row within planes 0 .. B-1
      const float4 L = *reinterpret_cast<const float4*>(disp + row + x);
      const float4 R = *reinterpret_cast<const float4*>(disp + half + row + (w - 4 - x));
      float4 o;
      o.x = post_process_pixel(L.x, R.w, x, w);
      o.y = post_process_pixel(L.y, R.z, x + 1, w);
      o.z = post_process_pixel(L.z, R.y, x + 2, w);
      o.w = post_process_pixel(L.w, R.x, x + 3, w);
      *reinterpret_cast<float4*>(out + row + x) = o;
    }
  } else {
    for (long long i = blockIdx.x * (long long)kM2Threads + threadIdx.x; i < half; i += (long long)gridDim.x * kM2Threads) {
      const int x = (int)(i % w);
      out[i] = post_process_pixel(disp[i], disp[half + (i - x) + (w - 1 - x)], x, w);
    }
  }
}

// one output index of one axis (ratio = n / O in fp64): the two taps and the weight of the second
static __device__ __forceinline__ void bilinear_tap(int o, int n, double ratio, int* i0, int* i1, double* f) {
  const double s = ((double)o + 0.5) * ratio - 0.5;
  const double fl = floor(s);
  int a = (int)fl;
  double fr = s - fl;
  if (a < 0) {
    a = 0;
    fr = 0.0;
  }
  if (a >= n - 1) {
    a = n - 1;
    fr = 0.0;
  }
  *i0 = a;
  *i1 = min(a + 1, n - 1);
  *f = fr;
}

// blockIdx.y = image; a thread makes the outputs 4t .. 4t + 3 of the image's flat H_b * W_b elements (rows are not padded, so a group
// may run over a row end) and stores them as one float4 where out + out_off[b] is 16-byte aligned and the group is whole.
__global__ void __launch_bounds__(kM2Threads) bilinear_recip_ragged_kernel(const float* __restrict__ disp, int h, int w,
                                                                           const int* __restrict__ out_hw,
                                                                           const long long* __restrict__ out_off, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int H = out_hw[2 * b], W = out_hw[2 * b + 1];
  if (H <= 0 || W <= 0) return;
  const long long n = (long long)H * W;
  const float* src = disp + (long long)b * h * w;
  float* dst = out + out_off[b];
  const bool vec = aligned16(dst);
  const double ry = (double)h / (double)H, rx = (double)w / (double)W;
  const long long groups = (n + 3) >> 2;
  for (long long t = blockIdx.x * (long long)kM2Threads + threadIdx.x; t < groups; t += (long long)gridDim.x * kM2Threads) {
    const long long e0 = t << 2;
    int y = (int)(e0 / W), x = (int)(e0 % W);
    int y0, y1;
    double fy;
    bilinear_tap(y, h, ry, &y0, &y1, &fy);
    float v[4];
    const int cnt = (int)(n - e0 < 4 ? n - e0 : 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = 0.f;
      if (k < cnt) {
        int x0, x1;
        double fx;
        bilinear_tap(x, w, rx, &x0, &x1, &fx);
        const float* r0 = src + (long long)y0 * w;
        const float* r1 = src + (long long)y1 * w;
        const double top = (1.0 - fx) * (double)r0[x0] + fx * (double)r0[x1];
        const double bot = (1.0 - fx) * (double)r1[x0] + fx * (double)r1[x1];
        v[k] = (float)(1.0 / ((1.0 - fy) * top + fy * bot));
        if (++x == W) {
          x = 0;
          ++y;
          if (k + 1 < cnt) bilinear_tap(y, h, ry, &y0, &y1, &fy);
        }
      }
    }
    if (vec && cnt == 4) {
      *reinterpret_cast<float4*>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int k = 0; k < cnt; ++k) dst[e0 + k] = v[k];
    }
  }
}

__global__ void __launch_bounds__(kErrThreads) eval_errors_clamp_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                                        const uint8_t* __restrict__ mask, const long long* __restrict__ off,
                                                                        const int* __restrict__ npix, int scale_mode, float fixed_scale,
                                                                        float lo, float hi, float* __restrict__ out) {
  eval_errors_image<true>(gt, pred, mask, off, npix, scale_mode, fixed_scale, lo, hi, out);
}

static inline unsigned m2_blocks(long long work) {
  long long b = (work + kM2Threads - 1) / kM2Threads;
  return (unsigned)(b < 1 ? 1 : (b > kM2MaxBlocks ? kM2MaxBlocks : b));
}

}  // namespace dn

using namespace dn;

extern "C" {

int dn_mono2_post_process(const float* disp, int32_t B, int32_t h, int32_t w, float* out, dn_stream_t stream) {
  DN_REQUIRE(disp && out && disp != out && B > 0 && h > 0 && w >= 2, DN_ERR_BAD_ARG, "dn_mono2_post_process: bad argument (w >= 2, not in place)");
  const long long half = (long long)B * h * w;
  if ((w & 3) == 0 && (reinterpret_cast<uintptr_t>(disp) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    DN_LAUNCH(mono2_post_process_kernel<true>, dim3(m2_blocks(half >> 2)), dim3(kM2Threads), 0, as_stream(stream), disp, (int)B, (int)h, (int)w,
              out);
  } else {
    DN_LAUNCH(mono2_post_process_kernel<false>, dim3(m2_blocks(half)), dim3(kM2Threads), 0, as_stream(stream), disp, (int)B, (int)h, (int)w, out);
  }
  return check_launch("mono2_post_process_kernel");
}

int dn_bilinear_recip_ragged(const float* disp, int32_t B, int32_t h, int32_t w, const int32_t* out_hw, const int64_t* out_off, int32_t max_h,
                             int32_t max_w, float* out, dn_stream_t stream) {
  DN_REQUIRE(disp && out_hw && out_off && out && B > 0 && B <= 65535 && h > 0 && w > 0 && max_h > 0 && max_w > 0, DN_ERR_BAD_ARG,
             "dn_bilinear_recip_ragged: bad argument");
  DN_REQUIRE((long long)max_h * max_w <= 0x7FFFFFFFLL, DN_ERR_UNSUPPORTED, "dn_bilinear_recip_ragged: %d x %d outputs per image are too many",
             (int)max_h, (int)max_w);
  const long long groups = ((long long)max_h * max_w + 3) >> 2;
  DN_LAUNCH(bilinear_recip_ragged_kernel, dim3(m2_blocks(groups), (unsigned)B), dim3(kM2Threads), 0, as_stream(stream), disp, (int)h, (int)w,
            (const int*)out_hw, (const long long*)out_off, out);
  return check_launch("bilinear_recip_ragged_kernel");
}

int dn_eval_errors_clamp(const float* gt, const float* pred, const uint8_t* mask, const int64_t* off, const int32_t* npix, int32_t B,
                         int32_t scale_mode, float fixed_scale, float lo, float hi, float* out, dn_stream_t stream) {
  DN_REQUIRE(gt && pred && mask && off && npix && out && B > 0, DN_ERR_BAD_ARG, "dn_eval_errors_clamp: bad argument");
  DN_REQUIRE(scale_mode >= 0 && scale_mode <= 2, DN_ERR_BAD_ARG, "dn_eval_errors_clamp: bad scale_mode %d", (int)scale_mode);
  DN_REQUIRE(lo > 0.f && lo <= hi, DN_ERR_BAD_ARG, "dn_eval_errors_clamp: bad clamp bounds [%g, %g]", (double)lo, (double)hi);
  DN_LAUNCH(eval_errors_clamp_kernel, dim3((unsigned)B), dim3(kErrThreads), 0, as_stream(stream), gt, pred, mask, (const long long*)off,
            (const int*)npix, (int)scale_mode, fixed_scale, lo, hi, out);
  return check_launch("eval_errors_clamp_kernel");
}

}  // extern "C"
