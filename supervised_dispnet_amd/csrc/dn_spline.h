// Cubic B-spline pieces shared by the NYU input chain (dn_nyu.hip) and the evaluation zoom (dn_eval.hip): scipy.ndimage's pole and
// per-line gain, its prefilter recurrences along a strided column and along a line held in LDS, its mirror index and its form of the
// four tap weights.  Both files compile with fp-contract off, which covers these helpers (the pragma is repeated here for them).
#pragma once

#pragma clang fp contract(off)

namespace dn {

constexpr double kPole = -0x1.126145e9ecd58p-2;    // sqrt(3) - 2 in fp64
constexpr double kGain = 0x1.7fffffffffffep+2;     // (1 - z) * (1 - 1/z) as scipy evaluates it (one line's gain)

static __device__ __forceinline__ int mirror_idx(int i, int n) {
  i = i < 0 ? -i : i;
  return i > n - 1 ? 2 * (n - 1) - i : i;
}

// cubic B-spline weights of the four taps floor(x)-1 .. floor(x)+2 at fraction t (scipy's form, last weight = 1 - the others)
static __device__ __forceinline__ void cubic_weights(double t, double* w) {
  const double z = 1.0 - t;
  w[0] = z * z * z / 6.0;
  w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
}

// scipy's prefilter of one line (mirror boundaries) -- gain, mirror causal init, causal pass, anti-causal init, anti-causal pass --
// from a strided fp32 column src[i * stride] into the fp64 column dst[i * stride].  The causal init needs every element: they are read
// from the source with the gain applied on the fly; the running value stays in a register; the causal values of 8 rows are loaded
// before the dependent anti-causal chain walks them.
static __device__ __forceinline__ void spline_prefilter_column(const float* __restrict__ src, double* __restrict__ dst, int H, long long stride) {
  const double z = kPole;
  const double z_n_1 = pow(z, (double)(H - 1));
  double c0 = (double)src[0] * kGain + z_n_1 * ((double)src[(long long)(H - 1) * stride] * kGain);
  double z_i = z;
#pragma unroll 8
  for (int i = 1; i < H - 1; ++i) {
    c0 += z_i * ((double)src[(long long)i * stride] * kGain + z_n_1 * ((double)src[(long long)(H - 1 - i) * stride] * kGain));
    z_i *= z;
  }
  double prev = c0 / (1.0 - z_n_1 * z_n_1);
  dst[0] = prev;
  double before_last = prev;
#pragma unroll 8
  for (int i = 1; i < H; ++i) {
    const double v = (double)src[(long long)i * stride] * kGain + z * prev;
    if (i == H - 2) before_last = v;
    dst[(long long)i * stride] = v;
    prev = v;
  }
  double next = (z * before_last + prev) * z / (z * z - 1.0);
  dst[(long long)(H - 1) * stride] = next;
  int i = H - 2;
  for (; i >= 7; i -= 8) {
    double d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = dst[(long long)(i - k) * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      next = z * (next - d[k]);
      dst[(long long)(i - k) * stride] = next;
    }
  }
  for (; i >= 0; --i) {
    next = z * (next - dst[(long long)i * stride]);
    dst[(long long)i * stride] = next;
  }
}

// the same recurrences in place on a contiguous line of n doubles (in LDS); the gain is applied where a value is first read
static __device__ __forceinline__ void spline_prefilter_line(double* c, int n) {
  const double z = kPole;
  const double z_n_1 = pow(z, (double)(n - 1));
  double c0 = c[0] * kGain + z_n_1 * (c[n - 1] * kGain);
  double z_i = z;
#pragma unroll 8
  for (int i = 1; i < n - 1; ++i) {
    c0 += z_i * (c[i] * kGain + z_n_1 * (c[n - 1 - i] * kGain));
    z_i *= z;
  }
  double p = c0 / (1.0 - z_n_1 * z_n_1);
  c[0] = p;
  double before_last = p;
#pragma unroll 8
  for (int i = 1; i < n; ++i) {
    p = c[i] * kGain + z * p;
    if (i == n - 2) before_last = p;
    c[i] = p;
  }
  p = (z * before_last + p) * z / (z * z - 1.0);
  c[n - 1] = p;
#pragma unroll 8
  for (int i = n - 2; i >= 0; --i) {
    p = z * (p - c[i]);
    c[i] = p;
  }
}

}  // namespace dn
